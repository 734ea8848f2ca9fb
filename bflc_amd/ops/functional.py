"""Op dispatch: hand-written gfx950 HIP kernels on GPU, torch fp32 on CPU.

Every numeric op of the reference's computational contract
(matmul+bias forward `main.py:120`, softmax-CE loss
`main.py:123`, SGD backward/update `main.py:127-130`, delta/candidate
AXPY `main.py:153-154,215-216`, argmax accuracy `main.py:182-183`,
weighted FedAvg `CommitteePrecompiled.cpp:373-414`) is owned here.

Dispatch rule (no silent fallbacks): tensors on a CUDA (ROCm) device
*must* go through the in-tree `bflc_amd._hip_ops` extension — if it is
missing the op raises instead of falling back to eager PyTorch. CPU
tensors use plain fp32 torch ops; they are the numerics oracle the GPU
kernels are tested against.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

_hip = None
_hip_err: Optional[str] = None


def _load_hip():
    global _hip, _hip_err
    if _hip is not None or _hip_err is not None:
        return _hip
    try:
        from bflc_amd import _hip_ops  # built in-tree by bflc_amd/build.py
        _hip = _hip_ops
    except ImportError as e:  # remember why, so the error is informative
        _hip_err = str(e)
    return _hip


def hip_ops():
    """The HIP extension, mandatory on GPU paths."""
    m = _load_hip()
    if m is None:
        raise RuntimeError(
            "bflc_amd._hip_ops (gfx950 HIP kernels) is not built/importable "
            f"({_hip_err}); run `python -m bflc_amd.build`. GPU execution "
            "without the native kernels is disabled by design.")
    return m


def hip_available() -> bool:
    return _load_hip() is not None


# ---------------------------------------------------------------------------
# autograd-wrapped primitives
# ---------------------------------------------------------------------------

class _LinearFn(torch.autograd.Function):
    """y = x @ w + b  (reference main.py:120: tf.matmul(x, W) + b).

    GPU: MFMA-tiled bf16 GEMM with fused bias epilogue + transpose-GEMM
    backward (csrc/hip/gemm_bf16.hip). CPU: torch fp32 oracle.
    """

    @staticmethod
    def forward(ctx, x: torch.Tensor, w: torch.Tensor, b: torch.Tensor,
                relu: bool):
        ctx.relu = relu
        if x.is_cuda:
            y = hip_ops().linear_fwd(x, w, b, relu)
        else:
            y = torch.addmm(b, x, w)
            if relu:
                y = torch.relu(y)
        ctx.save_for_backward(x, w, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        x, w, y = ctx.saved_tensors
        dy = dy.contiguous()
        if ctx.relu:  # fused-relu epilogue: mask dy by the saved output
            dy = hip_ops().relu_bwd(y, dy) if x.is_cuda \
                else dy * (y > 0).to(dy.dtype)
        # first-layer linears (logreg/MLP on raw features) need no
        # input gradient — skip the dx GEMM
        want_dx = ctx.needs_input_grad[0]
        if x.is_cuda:
            dx, dw, db = hip_ops().linear_bwd(x, w, dy, want_dx)
            if not want_dx:
                dx = None
        else:
            dx = dy @ w.t() if want_dx else None
            dw = x.t() @ dy
            db = dy.sum(0)
        return dx, dw, db, None


def linear(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor,
           relu: bool = False) -> torch.Tensor:
    return _LinearFn.apply(x, w, b, relu)


class _SoftmaxCEFn(torch.autograd.Function):
    """mean softmax cross-entropy over int labels, fused fwd+bwd
    (reference main.py:123). Returns scalar mean loss; backward produces
    dlogits = (softmax - onehot) * gscale / N computed in one kernel."""

    @staticmethod
    def forward(ctx, logits: torch.Tensor, target: torch.Tensor):
        if logits.is_cuda:
            loss, probs = hip_ops().softmax_ce_fwd(logits, target)
        else:
            lse = torch.logsumexp(logits.float(), dim=1)
            picked = logits.float().gather(1, target.view(-1, 1)).squeeze(1)
            loss = (lse - picked).mean()
            probs = torch.softmax(logits.float(), dim=1)
        ctx.save_for_backward(probs, target)
        ctx.in_dtype = logits.dtype
        return loss

    @staticmethod
    def backward(ctx, gloss: torch.Tensor):
        probs, target = ctx.saved_tensors
        if probs.is_cuda:
            dlogits = hip_ops().softmax_ce_bwd(probs, target, gloss)
        else:
            n = probs.shape[0]
            dlogits = probs.clone()
            dlogits.scatter_add_(
                1, target.view(-1, 1),
                torch.full((n, 1), -1.0, dtype=probs.dtype))
            dlogits = dlogits * (gloss / n)
        return dlogits.to(ctx.in_dtype), None


def softmax_cross_entropy(logits: torch.Tensor,
                          target: torch.Tensor) -> torch.Tensor:
    return _SoftmaxCEFn.apply(logits, target)


class _ReluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor):
        if x.is_cuda:
            y = hip_ops().relu_fwd(x)
        else:
            y = torch.relu(x)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        (y,) = ctx.saved_tensors
        if y.is_cuda:
            return hip_ops().relu_bwd(y, dy.contiguous())
        return dy * (y > 0).to(dy.dtype)


def relu(x: torch.Tensor) -> torch.Tensor:
    return _ReluFn.apply(x)


class _Conv2dFn(torch.autograd.Function):
    """NHWC conv (csrc/hip/conv2d.hip): channels-last makes 1x1 convs
    pure MFMA GEMMs (no im2col) and RxS gathers 16-B vector copies.
    x [N, H, W, C], w [Kout, R, S, C], y [N, OH, OW, Kout]. CPU oracle:
    permute to NCHW, torch fp32 conv, permute back."""

    @staticmethod
    def forward(ctx, x, w, b, stride: int, padding: int, relu: bool,
                want_col: bool):
        # NOTE: want_col is computed by the conv2d() wrapper OUTSIDE
        # this method — autograd.Function.forward always runs with grad
        # mode disabled internally, so torch.is_grad_enabled() in here
        # is unconditionally False
        ctx.stride, ctx.padding = stride, padding
        ctx.has_bias = b is not None
        ctx.relu = relu
        if x.is_cuda:
            y, col = hip_ops().conv2d_fwd_col(
                x, w, b if b is not None else
                torch.zeros(w.shape[0], device=x.device, dtype=x.dtype),
                stride, padding, relu, want_col)
            # keep col for wgrad when the fwd materialized one (the
            # implicit-GEMM path returns an empty marker; bwd then
            # builds its own)
            ctx.save_for_backward(x, w, col, y if relu else None)
            return y
        y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), b,
                     stride=stride, padding=padding)
        y = y.permute(0, 2, 3, 1).contiguous()
        if relu:
            y = torch.relu(y)
        ctx.save_for_backward(x, w, None, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors[:2]
        dy = dy.contiguous()
        db_fused = None
        if ctx.relu:  # fused-relu epilogue: mask dy by the saved output
            y = ctx.saved_tensors[3]
            if x.is_cuda and ctx.has_bias and w.shape[0] % 8 == 0:
                # one pass: mask dy AND accumulate db (was relu_bwd +
                # a full re-read of dy in colsum — ~10% of a FEMNIST
                # c1 round together)
                dy, db_fused = hip_ops().relu_bwd_colsum(y, dy)
            elif x.is_cuda:
                dy = hip_ops().relu_bwd(y, dy)
            else:
                dy = dy * (y > 0).to(dy.dtype)
        # first-layer convs (x = input data, no grad needed) skip the
        # entire dgrad GEMM + col2im — the ResNet-50 stem's dcol alone
        # is M x 147 (~236 MB) per backward
        want_dx = ctx.needs_input_grad[0]
        if x.is_cuda:
            col = ctx.saved_tensors[2]
            if col.numel() == 0:
                col = None
            dx, dw, db = hip_ops().conv2d_bwd(
                x, w, dy, ctx.stride, ctx.padding, col,
                ctx.has_bias and db_fused is None, want_dx)
            if not want_dx:
                dx = None
            if db_fused is not None:
                db = db_fused
            elif not ctx.has_bias:
                db = None
        else:
            xn = x.permute(0, 3, 1, 2)
            wn = w.permute(0, 3, 1, 2)
            dyn = dy.permute(0, 3, 1, 2)
            dx = None
            if want_dx:
                dx = torch.nn.grad.conv2d_input(
                    xn.shape, wn, dyn, stride=ctx.stride,
                    padding=ctx.padding)
                dx = dx.permute(0, 2, 3, 1).contiguous()
            dw = torch.nn.grad.conv2d_weight(
                xn, wn.shape, dyn, stride=ctx.stride, padding=ctx.padding)
            dw = dw.permute(0, 2, 3, 1).contiguous()
            db = dy.sum(dim=(0, 1, 2))
        return dx, dw, (db if ctx.has_bias else None), None, None, None, \
            None


def conv2d(x, w, b=None, stride: int = 1, padding: int = 0,
           relu: bool = False) -> torch.Tensor:
    # grad-free forwards (committee scoring / sponsor eval) skip the
    # col materialization entirely — thin shapes gather the window
    # inside the GEMM (gemm_thin_conv_kernel), identical output, no
    # 2x O(M*RSC) col traffic. Evaluated HERE (outside the Function:
    # forward() always executes with grad mode off).
    # Training also skips the col cache by default since the round-2
    # A/B: the backward's implicit wgrad route (Kout <= 64) beat the
    # materialize-in-forward-and-reuse design on MI355X (FEMNIST c1
    # 2.40 -> 2.36 ms/round) — 288 GB of HBM made caching free, but
    #8 TB/s makes NOT writing it faster. BFLC_CONV_NO_COL=0 restores
    # the cache for A/B.
    import os
    no_col = os.environ.get("BFLC_CONV_NO_COL", "1") == "1"
    want_col = (not no_col) and torch.is_grad_enabled() and \
        (x.requires_grad or w.requires_grad)
    return _Conv2dFn.apply(x, w, b, stride, padding, relu, want_col)


class _MaxPool2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel: int, stride: int, want_idx: bool):
        # want_idx comes from the maxpool2d() wrapper (grad mode is
        # always off inside Function.forward)
        if x.is_cuda:
            y, idx = hip_ops().maxpool2d_fwd(x, kernel, stride, want_idx)
        else:
            y, idx = F.max_pool2d(x.permute(0, 3, 1, 2), kernel, stride,
                                  return_indices=True)
            y = y.permute(0, 2, 3, 1).contiguous()
        ctx.save_for_backward(idx)
        ctx.in_shape = x.shape
        ctx.kernel, ctx.stride = kernel, stride
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        dy = dy.contiguous()
        if dy.is_cuda:
            dx = hip_ops().maxpool2d_bwd(dy, idx, list(ctx.in_shape),
                                         ctx.kernel, ctx.stride)
        else:
            dx = F.max_unpool2d(dy.permute(0, 3, 1, 2), idx, ctx.kernel,
                                ctx.stride,
                                output_size=ctx.in_shape[1:3])
            dx = dx.permute(0, 2, 3, 1).contiguous()
        return dx, None, None, None


def maxpool2d(x, kernel: int = 2, stride: Optional[int] = None) -> torch.Tensor:
    want_idx = torch.is_grad_enabled() and x.requires_grad
    return _MaxPool2dFn.apply(x, kernel, stride or kernel, want_idx)


class _ConvReluPoolFn(torch.autograd.Function):
    """Training conv + bias + ReLU + 2x2/2 maxpool on the fused GPU
    routes (csrc/hip/conv2d.hip). The forward pools in the conv
    epilogue and also emits the u8 argmax plane; only (x, w, y_pooled,
    idx) are saved — the full-resolution activation never exists. The
    backward unpools, ReLU-masks by y_pooled > 0 and sums db in one
    pass, then runs the unchanged conv backward (for a thin first layer
    the same MFMA chains fed straight from the pooled tensors, see
    thin_conv_pool_wgrad_fused; for conv2 at an unsplit batch the data
    gradient comes from halo_pool_dgrad_kernel, which unpools into LDS,
    leaves the plane behind for the weight gradient and reads w without
    the permuted copy, see pool_dgrad_impl): every gradient is bitwise
    the two-op path's. With direct_wgrad (BFLC_THIN_DIRECT_WGRAD
    =1) a thin first layer goes straight to (dw, db) instead, which is
    faster but sums them in its own order (last-bit differences)."""

    @staticmethod
    def forward(ctx, x, w, b, stride: int, padding: int,
                direct_wgrad: bool):
        ctx.stride, ctx.padding = stride, padding
        ctx.direct_wgrad = direct_wgrad
        ctx.has_bias = b is not None
        bias = b if b is not None else torch.zeros(
            w.shape[0], device=x.device, dtype=x.dtype)
        y, idx = hip_ops().conv2d_relu_pool_fwd_idx(x, w, bias, stride,
                                                    padding)
        ctx.save_for_backward(x, w, y, idx)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y, idx = ctx.saved_tensors
        want_dx = ctx.needs_input_grad[0]
        dx, dw, db = hip_ops().conv2d_relu_pool_bwd(
            x, w, y, idx, dy.contiguous(), ctx.stride, ctx.padding,
            ctx.has_bias, want_dx, ctx.direct_wgrad)
        return (dx if want_dx else None, dw,
                db if ctx.has_bias else None, None, None, None)


def conv2d_relu_pool(x, w, b=None, stride: int = 1,
                     padding: int = 0) -> torch.Tensor:
    """maxpool2d(conv2d(x, w, b, relu=True), 2).

    On a GPU the 2x2 pool runs in the conv kernel's epilogue wherever a
    fused route takes the shape, so the full-resolution activation is
    never written to HBM and re-read; the pooled result is bitwise the
    two-op sequence (csrc/hip/conv2d.hip). With grad mode off
    (committee scoring, sponsor eval) that is the whole op. With grad
    mode on, _ConvReluPoolFn additionally keeps the argmax plane and
    runs the fused backward, whose gradients are bitwise the two-op
    ones; BFLC_THIN_DIRECT_WGRAD=1 opts the thin first layer into the
    direct weight-gradient kernel (faster, but dW/db of that layer may
    move in the last bit). The CPU, shapes no fused route takes, and
    either gate switched off keep the two-op autograd sequence. The
    grad-mode test sits here, not in a Function.forward (which always
    runs with grad mode off). BFLC_FUSED_POOL=0 restores the two-op
    eval path and BFLC_FUSED_POOL_TRAIN=0 the two-op training path for
    A/B runs.
    """
    import os
    if x.is_cuda and not torch.is_grad_enabled() and \
            os.environ.get("BFLC_FUSED_POOL", "1") == "1":
        bias = b if b is not None else torch.zeros(
            w.shape[0], device=x.device, dtype=x.dtype)
        return hip_ops().conv2d_relu_pool_fwd(x, w, bias, stride, padding)
    if x.is_cuda and torch.is_grad_enabled() and \
            os.environ.get("BFLC_FUSED_POOL_TRAIN", "1") != "0" and \
            hip_ops().conv2d_relu_pool_route(
                list(x.shape), list(w.shape), stride, padding) != "unfused":
        return _ConvReluPoolFn.apply(
            x, w, b, stride, padding,
            os.environ.get("BFLC_THIN_DIRECT_WGRAD", "0") == "1")
    return maxpool2d(conv2d(x, w, b, stride, padding, relu=True), 2)


def conv_relu_pool_stack(x, w1, b1, w2, b2) -> torch.Tensor:
    """Two conv3x3(stride 1, pad 1) + ReLU + 2x2 pool stages:
    conv2d_relu_pool(conv2d_relu_pool(x, w1, b1, 1, 1), w2, b2, 1, 1).

    With grad mode off, on a GPU, where conv_relu_pool_stack_route says
    "halo_stack" (a thin first layer into the halo-tile second one, see
    csrc/hip/halo_conv.hip) the pair is ONE kernel: each block computes
    its conv2 input images from the raw pixels straight into LDS, so the
    pooled first-layer activation is never written to HBM and read back.
    The result is bitwise the two calls. Training, the CPU, every other
    shape and BFLC_FUSED_POOL=0 run the two calls; BFLC_HALO_STACK=0
    (read once per process) closes the route for A/B runs.
    """
    import os
    if x.is_cuda and not torch.is_grad_enabled() and \
            os.environ.get("BFLC_FUSED_POOL", "1") == "1" and \
            b1 is not None and b2 is not None and \
            hip_ops().conv_relu_pool_stack_route(
                list(x.shape), list(w1.shape), list(w2.shape)) == "halo_stack":
        return hip_ops().conv_relu_pool_stack_fwd(x, w1, b1, w2, b2, 0, "")
    h = conv2d_relu_pool(x, w1, b1, 1, 1)
    return conv2d_relu_pool(h, w2, b2, 1, 1)


class _BatchNormFn(torch.autograd.Function):
    """BatchNorm2d (NHWC, batch-stats mode: train AND eval — no running
    buffers; the FedBN-style simplification so the flat parameter vector
    is exactly {gamma, beta}). GPU: column-reduction kernels over
    x viewed [N*H*W, C] (csrc/hip/batchnorm.hip); CPU: fp32 oracle."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps: float, relu: bool, residual):
        if x.is_cuda:
            y, mean, invstd = hip_ops().batchnorm_fwd(x, gamma, beta, eps,
                                                      relu, residual)
        else:
            xf = x.float()
            mean = xf.mean(dim=(0, 1, 2))
            var = xf.var(dim=(0, 1, 2), unbiased=False)
            invstd = (var + eps).rsqrt()
            y = (xf - mean) * invstd * gamma.float() + beta.float()
            if residual is not None:
                y = y + residual.float()
            if relu:
                y = torch.relu(y)
            y = y.to(x.dtype)
        ctx.relu = relu
        ctx.has_res = residual is not None
        if relu:
            ctx.save_for_backward(x, gamma, mean, invstd, y)
        else:
            ctx.save_for_backward(x, gamma, mean, invstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, invstd = ctx.saved_tensors[:4]
        yr = ctx.saved_tensors[4] if ctx.relu else None
        dy = dy.contiguous()
        dres = None
        if x.is_cuda:
            if ctx.has_res:
                # residual grad = relu-masked dy (same mask BN bwd uses)
                dres = (hip_ops().add_relu_bwd(yr, dy) if yr is not None
                        else dy)
            dx, dgamma, dbeta = hip_ops().batchnorm_bwd(x, dy, mean, invstd,
                                                        gamma, yr)
        else:
            xf, dyf = x.float(), dy.float()
            if yr is not None:
                dyf = dyf * (yr.float() > 0)
            if ctx.has_res:
                dres = dyf.to(x.dtype)
            n = x.numel() / x.shape[-1]
            xhat = (xf - mean) * invstd
            sdy = dyf.sum(dim=(0, 1, 2))
            sdyx = (dyf * xhat).sum(dim=(0, 1, 2))
            dx = (gamma.float() * invstd) * (dyf - sdy / n - xhat * sdyx / n)
            dx = dx.to(x.dtype)
            dgamma = sdyx.to(x.dtype)
            dbeta = sdy.to(x.dtype)
        return dx, dgamma, dbeta, None, None, dres


class _ConvBNFn(torch.autograd.Function):
    """Fused conv + batch-stats BN (+relu, +residual) for the GPU path:
    the conv GEMM's epilogue emits per-tile channel partials, one tiny
    fixed-tree kernel finalizes mean/invstd, and a single normalization
    pass produces the block output — the standalone BN stats sweep over
    the conv activation disappears. Backward = BN backward (relu mask
    folded into its reductions) then conv backward."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, stride, padding, eps, relu,
                residual):
        h = hip_ops()
        ctx.stride, ctx.padding, ctx.relu = stride, padding, relu
        ctx.has_res = residual is not None
        yc, col, psum, psq = h.conv2d_fwd_bn(x, w, stride, padding)
        M = yc.numel() // yc.shape[-1]
        if psum.numel() > 0:
            mean, invstd = h.bn_stats_finalize(psum, psq, float(M), eps)
        else:  # split-K / unsupported shape: standalone stats pass
            mean, invstd = h.bn_stats(yc, eps)
        y = h.batchnorm_norm(yc, gamma, beta, mean, invstd, relu, residual)
        saved = [x, w, col, yc, gamma, mean, invstd]
        if relu:
            saved.append(y)
        ctx.save_for_backward(*saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        h = hip_ops()
        x, w, col, yc, gamma, mean, invstd = ctx.saved_tensors[:7]
        yr = ctx.saved_tensors[7] if ctx.relu else None
        dy = dy.contiguous()
        dres = None
        if ctx.has_res:
            dres = h.add_relu_bwd(yr, dy) if yr is not None else dy
        dyc, dgamma, dbeta = h.batchnorm_bwd(yc, dy, mean, invstd, gamma,
                                             yr)
        # want_db=False: the BN absorbs any bias, so no colsum pass over
        # dyc (it was ~3.3% of a ResNet-20 round for a discarded value).
        # want_dx=False on the stem (x = input images): skips the dgrad
        # GEMM + col2im entirely.
        want_dx = ctx.needs_input_grad[0]
        dx, dw, _db = h.conv2d_bwd(x, w, dyc, ctx.stride, ctx.padding,
                                   col if col.numel() > 0 else None,
                                   False, want_dx)
        if not want_dx:
            dx = None
        return (dx, dw, dgamma, dbeta, None, None, None, None, dres)


def conv2d_bn(x, w, gamma, beta, stride: int = 1, padding: int = 0,
              eps: float = 1e-5, relu: bool = True,
              residual=None) -> torch.Tensor:
    """conv2d (no bias) -> batch-stats BN -> optional residual+relu,
    fused on GPU (epilogue stats + single norm pass); on CPU the
    composition of the fp32 oracle ops."""
    if not x.is_cuda:
        return batchnorm2d(conv2d(x, w, None, stride, padding), gamma,
                           beta, eps, relu, residual)
    return _ConvBNFn.apply(x, w, gamma, beta, stride, padding, eps, relu,
                           residual)


def batchnorm2d(x, gamma, beta, eps: float = 1e-5, relu: bool = False,
                residual=None) -> torch.Tensor:
    """Batch-stats BN with optionally FUSED residual add + relu (one
    kernel fwd; the relu mask folds into the backward reductions and
    the residual grad is the masked dy)."""
    return _BatchNormFn.apply(x, gamma, beta, eps, relu, residual)


class _GroupNormFn(torch.autograd.Function):
    """GroupNorm (NHWC): statistics per (sample, group) over H*W*C/G
    elements, so a sample's output does not depend on the rest of its
    batch; parameters are the same per-channel {gamma, beta} as BN.
    GPU: csrc/hip/groupnorm.hip (slab / split routes, chosen from
    (H, W, C, G) only); CPU: fp32 oracle. Any shape on CPU; the GPU
    kernels need C % 8 == 0 and raise otherwise."""

    @staticmethod
    def forward(ctx, x, gamma, beta, groups: int, eps: float, relu: bool,
                residual):
        if x.is_cuda:
            y, mean, rstd = hip_ops().groupnorm_fwd(x, gamma, beta, groups,
                                                    eps, relu, residual)
        else:
            N, H, W, C = x.shape
            if groups <= 0 or C % groups:
                raise ValueError(f"groupnorm: C={C} is not divisible by "
                                 f"groups={groups}")
            xg = x.float().reshape(N, H * W, groups, C // groups)
            mean = xg.mean(dim=(1, 3))
            var = xg.var(dim=(1, 3), unbiased=False)
            rstd = (var + eps).rsqrt()
            xhat = ((xg - mean[:, None, :, None]) * rstd[:, None, :, None]) \
                .reshape(N, H, W, C)
            y = xhat * gamma.float() + beta.float()
            if residual is not None:
                y = y + residual.float()
            if relu:
                y = torch.relu(y)
            y = y.to(x.dtype)
        ctx.groups = groups
        ctx.relu = relu
        ctx.has_res = residual is not None
        if relu:
            ctx.save_for_backward(x, gamma, mean, rstd, y)
        else:
            ctx.save_for_backward(x, gamma, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, rstd = ctx.saved_tensors[:4]
        yr = ctx.saved_tensors[4] if ctx.relu else None
        dy = dy.contiguous()
        dres = None
        G = ctx.groups
        if x.is_cuda:
            if ctx.has_res:
                # residual grad = relu-masked dy (same mask GN bwd uses)
                dres = (hip_ops().add_relu_bwd(yr, dy) if yr is not None
                        else dy)
            dx, dgamma, dbeta = hip_ops().groupnorm_bwd(x, dy, mean, rstd,
                                                        gamma, G, yr)
        else:
            N, H, W, C = x.shape
            dyf = dy.float()
            if yr is not None:
                dyf = dyf * (yr.float() > 0)
            if ctx.has_res:
                dres = dyf.to(x.dtype)
            m = H * W * (C // G)
            xg = x.float().reshape(N, H * W, G, C // G)
            xhat = (xg - mean[:, None, :, None]) * rstd[:, None, :, None]
            d = (dyf * gamma.float()).reshape(N, H * W, G, C // G)
            sd = d.sum(dim=(1, 3), keepdim=True)
            sdx = (d * xhat).sum(dim=(1, 3), keepdim=True)
            dx = rstd[:, None, :, None] * (d - sd / m - xhat * sdx / m)
            dx = dx.reshape(N, H, W, C).to(x.dtype)
            xhat = xhat.reshape(N, H, W, C)
            dgamma = (dyf * xhat).sum(dim=(0, 1, 2)).to(x.dtype)
            dbeta = dyf.sum(dim=(0, 1, 2)).to(x.dtype)
        return dx, dgamma, dbeta, None, None, None, dres


def groupnorm2d(x, gamma, beta, groups: int, eps: float = 1e-5,
                relu: bool = False, residual=None) -> torch.Tensor:
    """Per-sample GroupNorm with optionally FUSED residual add + relu
    (one rounding to the output dtype; the relu mask folds into the
    backward reductions and the residual grad is the masked dy)."""
    return _GroupNormFn.apply(x, gamma, beta, int(groups), eps, relu,
                              residual)


def conv2d_gn(x, w, gamma, beta, groups: int, stride: int = 1,
              padding: int = 0, eps: float = 1e-5, relu: bool = True,
              residual=None) -> torch.Tensor:
    """conv2d (no bias) -> GroupNorm -> optional residual+relu. The BN
    path's epilogue-stats fusion emits whole-batch channel partials and
    cannot serve per-sample statistics, so the conv runs unfused;
    conv2d still skips the dgrad when x needs no gradient (the stem)."""
    return groupnorm2d(conv2d(x, w, None, stride, padding), gamma, beta,
                       groups, eps, relu, residual)


def groupnorm_route(H: int, W: int, C: int, groups: int) -> str:
    """'slab' or 'split': the route the GPU launcher takes for an
    activation [N, H, W, C] — a function of (H, W, C, groups) and the
    BFLC_GN_ROUTE knob only, never of N. Host code, needs no GPU."""
    return hip_ops().groupnorm_route(H, W, C, groups)


class _GlobalAvgPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.hw = (x.shape[1], x.shape[2])
        if x.is_cuda:
            return hip_ops().global_avgpool_fwd(x)
        return x.mean(dim=(1, 2))

    @staticmethod
    def backward(ctx, dy):
        h, w = ctx.hw
        dy = dy.contiguous()
        if dy.is_cuda:
            return hip_ops().global_avgpool_bwd(dy, h, w)
        return (dy / (h * w))[:, None, None, :].expand(-1, h, w, -1) \
            .contiguous()


def global_avgpool(x) -> torch.Tensor:
    return _GlobalAvgPoolFn.apply(x)


class _AddReluFn(torch.autograd.Function):
    """Fused residual add + relu (one kernel instead of two)."""

    @staticmethod
    def forward(ctx, a, b):
        if a.is_cuda:
            y = hip_ops().add_relu_fwd(a, b.contiguous())
        else:
            y = torch.relu(a + b)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = dy.contiguous()
        if y.is_cuda:
            da = hip_ops().add_relu_bwd(y, dy)
        else:
            da = dy * (y > 0).to(dy.dtype)
        return da, da


def add_relu(a, b) -> torch.Tensor:
    return _AddReluFn.apply(a, b)


# ---------------------------------------------------------------------------
# non-autograd FL math (flat-tensor ops)
# ---------------------------------------------------------------------------

def accuracy_t(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """mean(argmax(pred) == label) as a DEVICE tensor (no host sync) —
    fused argmax-compare-reduce kernel on GPU."""
    if logits.is_cuda:
        return hip_ops().accuracy_t(logits, target)
    return (logits.argmax(dim=1) == target).float().mean()


def accuracy(logits: torch.Tensor, target: torch.Tensor) -> float:
    """mean(argmax(pred) == label) — reference main.py:182-183."""
    return float(accuracy_t(logits, target))


def axpy_(y: torch.Tensor, alpha: float, x: torch.Tensor) -> torch.Tensor:
    """y += alpha * x in place (delta extraction / candidate
    reconstruction, reference main.py:153-154, 215-216)."""
    if y.is_cuda:
        hip_ops().axpy_(y, x, float(alpha))
        return y
    return y.add_(x, alpha=alpha)


def score_load_(shadow: torch.Tensor, global_flat: torch.Tensor,
                delta: torch.Tensor, lr: float) -> None:
    """shadow = compute_dtype(global - lr*delta) in ONE pass: the
    committee-scoring candidate load (reference candidate
    reconstruction, main.py:215-216). The scorer's forward reads only
    the compute-dtype shadow, so the fp32 master copy of set_flat is
    skipped entirely; fp32 math with one rounding — bitwise identical
    to the copy+axpy+set_flat chain it replaces."""
    if shadow.is_cuda:
        hip_ops().score_load_(shadow, global_flat, delta, float(lr))
    else:
        with torch.no_grad():
            shadow.copy_((global_flat - lr * delta).to(shadow.dtype))


def delta_extract_(out: torch.Tensor, global_flat: torch.Tensor,
                   w: torch.Tensor, lr: float) -> None:
    """out = (global - w)/lr in ONE pass: pseudo-gradient extraction
    (reference main.py:153-154), replacing clone + axpy + scalar-div.
    The quotient may differ from torch's reciprocal-multiply div_ by
    1 ulp; every rank runs the same kernel, so replicas stay
    bitwise-identical."""
    if out.is_cuda:
        hip_ops().delta_extract_(out, global_flat, w, float(lr))
    else:
        with torch.no_grad():
            torch.sub(global_flat, w, out=out)
            out.div_(lr)


def sgd_step_(flat_param: torch.Tensor, flat_grad: torch.Tensor,
              lr: float) -> None:
    """Fused flat SGD update (reference main.py:127-130)."""
    if flat_param.is_cuda:
        hip_ops().sgd_step_(flat_param, flat_grad, float(lr))
    else:
        flat_param.add_(flat_grad, alpha=-lr)


def grad_sumsq_geom(n: int):
    """(blocks, longest lane chain in elements, adds after the lane
    chain) of the sum-of-squares kernels at n elements — a function of n
    alone, answered by the extension's host code (no GPU needed)."""
    return tuple(hip_ops().grad_sumsq_geom(int(n)))


def sgdm_step_geom(n: int):
    """(blocks, threads, elements per thread per grid-stride pass) of
    the fused sgdm update at n elements (host code, no GPU needed)."""
    return tuple(hip_ops().sgdm_step_geom(int(n)))


def grad_clip_coef_(g: torch.Tensor, clip: float,
                    out: torch.Tensor) -> None:
    """out[0] = min(1, clip / (||g||_2 + 1e-6)) — the coefficient of
    torch.nn.utils.clip_grad_norm_ — as a DEVICE float (no host sync);
    0 when the sum of squares is not finite, which makes sgdm_step_ skip
    the step. out may hold a second float, which receives sum(g^2).

    GPU: grad_sumsq_part + grad_clip_final (csrc/hip/optimizer.hip),
    fp32 with a fixed summation order. CPU oracle: the same formula with
    an fp32 sum in torch's order."""
    if not clip > 0:
        raise ValueError("clip must be > 0")
    if g.is_cuda:
        hip_ops().grad_clip_coef_(g, float(clip), out)
        return
    with torch.no_grad():
        _clip_coef_cpu(g.float().square().sum(), clip, out)


def _clip_coef_cpu(ss: torch.Tensor, clip: float, out: torch.Tensor) -> None:
    if bool(torch.isfinite(ss)):
        coef = torch.clamp(
            torch.tensor(float(clip), dtype=torch.float32)
            / (ss.sqrt() + 1e-6), max=1.0)
    else:
        coef = torch.zeros((), dtype=torch.float32)
    out[0] = coef
    if out.numel() > 1:
        out[1] = ss


def grad_clip_final_(part: torch.Tensor, clip: float,
                     out: torch.Tensor) -> None:
    """grad_clip_coef_'s second half on per-block partials `part` of a
    sum of squares (written by delta_extract_sumsq_): out[0] = the clip
    coefficient, out[1] = the sum. Same kernel, so the same bits as
    grad_clip_coef_ on the stored vector."""
    if not clip > 0:
        raise ValueError("clip must be > 0")
    if part.is_cuda:
        hip_ops().grad_clip_final_(part, float(clip), out)
        return
    with torch.no_grad():
        _clip_coef_cpu(part.sum(), clip, out)


# ---------------------------------------------------------------------------
# differential privacy (csrc/hip/privacy.hip; DESIGN.md "Round-13")
# ---------------------------------------------------------------------------

DP_CENTRAL_STREAM = 0xFFFFFFFF   # noise stream of the aggregate
_M32 = 0xFFFFFFFF


def sumsq_partials(n: int, device) -> int:
    """Length of the `part` buffer delta_extract_sumsq_ needs for an
    n-element vector on `device` (the CPU oracle keeps the sum in
    part[0])."""
    if torch.device(device).type == "cuda":
        return grad_sumsq_geom(n)[0]
    return 1


def _philox4x32_10_np(ctr, key0: int, key1: int):
    """Philox4x32-10 on an [N, 4] array of 32-bit counters, in uint64
    numpy arithmetic (every product of two 32-bit words fits)."""
    import numpy as np
    c = [np.ascontiguousarray(ctr[:, j]).astype(np.uint64) & np.uint64(_M32)
         for j in range(4)]
    k0, k1 = int(key0) & _M32, int(key1) & _M32
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    mask, sh = np.uint64(_M32), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]
        c = [(p1 >> sh) ^ c[1] ^ np.uint64(k0), p1 & mask,
             (p0 >> sh) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0 = (k0 + 0x9E3779B9) & _M32
        k1 = (k1 + 0xBB67AE85) & _M32
    return np.stack(c, axis=1)


def _dp_normals_np(n: int, seed: int, stream: int, epoch: int):
    """z(0..n-1) of the noise definition as float64: coordinate i takes
    element i & 3 of the Box-Muller pairs of Philox block i >> 2."""
    import numpy as np
    nb = (n + 3) // 4
    b = np.arange(nb, dtype=np.uint64)
    ctr = np.stack([b & np.uint64(_M32), b >> np.uint64(32),
                    np.full(nb, int(stream) & _M32, dtype=np.uint64),
                    np.full(nb, int(epoch) & _M32, dtype=np.uint64)], axis=1)
    seed = int(seed)
    x = _philox4x32_10_np(ctr, seed & _M32, (seed >> 32) & _M32)
    u = ((x >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    r0 = np.sqrt(-2.0 * np.log(u[:, 0]))
    r1 = np.sqrt(-2.0 * np.log(u[:, 2]))
    a0, a1 = 2.0 * np.pi * u[:, 1], 2.0 * np.pi * u[:, 3]
    z = np.stack([r0 * np.cos(a0), r0 * np.sin(a0),
                  r1 * np.cos(a1), r1 * np.sin(a1)], axis=1)
    return z.reshape(-1)[:n]


def delta_extract_sumsq_(out: torch.Tensor, global_flat: torch.Tensor,
                         w: torch.Tensor, lr: float,
                         part: torch.Tensor) -> None:
    """delta_extract_ (same bits) and, in the same pass, the per-block
    partials of sum(out^2) into `part` (sumsq_partials elements), in
    grad_clip_coef_'s summation order: grad_clip_final_(part, clip, coef)
    then equals grad_clip_coef_(out, clip, coef) bitwise, one read pass
    over the vector cheaper. GPU tensors must be 16-byte aligned."""
    if out.is_cuda:
        hip_ops().delta_extract_sumsq_(out, global_flat, w, float(lr), part)
        return
    delta_extract_(out, global_flat, w, lr)
    with torch.no_grad():
        part.zero_()
        part[0] = out.float().square().sum()


def dp_privatize_(d: torch.Tensor, coef_dev: torch.Tensor, sigma: float,
                  seed: int, stream: int, epoch: int) -> None:
    """In place on a contiguous fp32 vector: d[i] = fmaf(coef, d[i], n_i)
    with n_i = fp32(sigma * z(i)) and z the standard normal of
    (seed, stream, epoch, i) — Philox4x32-10 on counter (i >> 2 lo,
    i >> 2 hi, stream, epoch) under key (seed lo, seed hi), words to
    u = ((x >> 8) + 0.5) * 2^-24, Box-Muller, element i & 3. `coef_dev`
    is a device float (grad_clip_final_'s output). coef == 0 (a
    non-finite update) publishes n_i alone; sigma == 0 is the clip alone,
    d[i] = coef * d[i], and runs no generator.

    The CPU oracle evaluates z in float64 and rounds once."""
    if not sigma >= 0:
        raise ValueError("sigma must be >= 0")
    seed, stream, epoch = int(seed), int(stream), int(epoch)
    if not (0 <= seed < 1 << 64 and 0 <= stream <= _M32
            and 0 <= epoch <= _M32):
        raise ValueError("seed is 64-bit, stream and epoch are 32-bit")
    if d.is_cuda:
        hip_ops().dp_privatize_(d, coef_dev, float(sigma), seed, stream,
                                epoch)
        return
    import numpy as np
    if d.dtype != torch.float32 or not d.is_contiguous():
        raise ValueError("d must be a contiguous fp32 tensor")
    with torch.no_grad():
        coef = np.float32(float(coef_dev[0]))
        sig = np.float32(sigma)
        dv = d.view(-1).numpy()
        if sig != 0:
            z = _dp_normals_np(dv.size, seed, stream, epoch)
            nz = sig * z.astype(np.float32)
        else:
            nz = np.zeros(dv.size, dtype=np.float32)
        if coef == 0:
            dv[:] = nz
        elif sig != 0:
            dv[:] = (np.float64(coef) * dv.astype(np.float64)
                     + nz.astype(np.float64)).astype(np.float32)
        else:
            dv[:] = coef * dv


def dp_philox_words(ctr: torch.Tensor, key0: int, key1: int) -> torch.Tensor:
    """Philox4x32-10 of the [N, 4] int64 counters (each a 32-bit value)
    under the 32-bit key words: [N, 4] int64 output words. On the GPU
    this runs the device function dp_privatize_ draws from."""
    key0, key1 = int(key0), int(key1)
    if not (0 <= key0 <= _M32 and 0 <= key1 <= _M32):
        raise ValueError("key words are 32-bit")
    if ctr.is_cuda:
        return hip_ops().dp_philox_words(ctr.contiguous(), key0, key1)
    import numpy as np
    x = _philox4x32_10_np(ctr.numpy().astype(np.uint64), key0, key1)
    return torch.from_numpy(x.astype(np.int64))


def sgdm_step_(p: torch.Tensor, shadow: Optional[torch.Tensor],
               g: torch.Tensor, buf: torch.Tensor, p0: torch.Tensor,
               lr_dev: torch.Tensor, coef_dev: torch.Tensor,
               momentum: float, nesterov: bool, wd: float,
               mu: float) -> None:
    """Fused extended-SGD update of the fp32 master `p` (and its bf16
    `shadow`, or None) in place; `lr_dev` and `coef_dev` are 1-element
    fp32 tensors on p's device, so a captured graph replays under a
    refilled learning rate.

    Operation order (identical in sgdm_master_dev_kernel,
    csrc/hip/optimizer.hip): every input is widened exactly to fp64, the
    chain runs in fp64, and p and buf are each rounded to fp32 once:

        if coef == 0: return          (non-finite gradient: step skipped)
        g = coef * grad               (the clip scales the loss gradient only)
        g = fma(wd, p, g)             only if wd != 0
        g = fma(mu, p - p0, g)        only if mu != 0 (p0 untouched otherwise)
        b = fma(mom, buf, g); buf = fp32(b)    only if momentum != 0
        d = nesterov ? fma(mom, b, g) : b      (d = g without momentum)
        p = fp32(fma(-lr, d, p)); shadow = bf16(p)

    The CPU oracle below evaluates the same chain with separate fp64
    multiply and add; against the kernel's fused fp64 fma that can move
    a stored fp32 value only when the fp64 result sits within 2^-53 of a
    rounding boundary. `buf` is read and written only at momentum != 0
    and `p0` read only at mu != 0 — pass any tensor otherwise."""
    if nesterov and not momentum > 0:
        raise ValueError("nesterov needs momentum > 0")
    if p.is_cuda:
        hip_ops().sgdm_master_dev_(p, shadow, g, buf, p0, lr_dev, coef_dev,
                                   float(momentum), bool(nesterov),
                                   float(wd), float(mu))
        return
    with torch.no_grad():
        coef = coef_dev[0].double()
        if float(coef) == 0.0:
            return
        pd = p.double()
        gd = coef * g.double()
        if wd != 0:
            gd = gd + float(wd) * pd
        if mu != 0:
            gd = gd + float(mu) * (pd - p0.double())
        d = gd
        if momentum != 0:
            b = float(momentum) * buf.double() + gd
            buf.copy_(b.float())
            d = gd + float(momentum) * b if nesterov else b
        p.copy_((pd - lr_dev[0].double() * d).float())
        if shadow is not None:
            shadow.copy_(p.to(shadow.dtype))


def adam_step_(flat_param: torch.Tensor, flat_grad: torch.Tensor,
               m: torch.Tensor, v: torch.Tensor, step: int, lr: float,
               beta1: float = 0.9, beta2: float = 0.999,
               eps: float = 1e-8) -> None:
    """Fused flat Adam update (reference main.py:126, present but
    commented out; provided as a first-class optimizer here)."""
    if flat_param.is_cuda:
        hip_ops().adam_step_(flat_param, flat_grad, m, v, int(step),
                             float(lr), float(beta1), float(beta2), float(eps))
    else:
        m.mul_(beta1).add_(flat_grad, alpha=1 - beta1)
        v.mul_(beta2).addcmul_(flat_grad, flat_grad, value=1 - beta2)
        mhat = m / (1 - beta1 ** step)
        vhat = v / (1 - beta2 ** step)
        flat_param.addcdiv_(mhat, vhat.sqrt().add_(eps), value=-lr)


def weighted_fedavg(deltas: torch.Tensor, weights: torch.Tensor
                    ) -> torch.Tensor:
    """avg[i] = sum_k w[k]*deltas[k,i] / sum_k w[k] with a FIXED k-order
    accumulation so every rank computes bit-identical aggregates
    (reference CommitteePrecompiled.cpp:373-400). deltas: [K, P] fp32,
    weights: [K] fp32. One weighted-reduce HIP kernel on GPU."""
    if deltas.is_cuda:
        return hip_ops().weighted_fedavg(deltas, weights)
    acc = torch.zeros(deltas.shape[1], dtype=torch.float32)
    for k in range(deltas.shape[0]):  # fixed order, matches the kernel
        acc += deltas[k].float() * weights[k]
    return acc / weights.sum()


# ---------------------------------------------------------------------------
# robust aggregation (csrc/hip/aggregate.hip): [K, P] fp32 stack, K <= 32
# ---------------------------------------------------------------------------

MAX_AGG_ROWS = 32


def _check_stack(deltas: torch.Tensor) -> None:
    if deltas.dim() != 2 or deltas.dtype != torch.float32:
        raise ValueError("deltas must be a [K, P] fp32 tensor")
    K, P = deltas.shape
    if not 1 <= K <= MAX_AGG_ROWS or P < 1:
        raise ValueError(f"need 1 <= K <= {MAX_AGG_ROWS} and P >= 1, got "
                         f"K={K} P={P}")


def order_stat_mean(deltas: torch.Tensor, t: int) -> torch.Tensor:
    """Per coordinate: sort the K values, drop `t` at each end, add the
    rest in ascending sorted order in fp32, divide in fp32 by K - 2t.
    Ordering is by value with every NaN above +inf, so up to t
    non-finite rows per coordinate are trimmed away and more propagate
    NaN. t = 0 is the unweighted mean, t = (K-1)//2 the median. Summing
    in sorted order makes the result bitwise invariant to row order.
    The CPU path is the oracle of the sort-network kernel."""
    _check_stack(deltas)
    K = deltas.shape[0]
    t = int(t)
    if t < 0 or 2 * t >= K:
        raise ValueError(f"need 0 <= 2t < K, got t={t} K={K}")
    if deltas.is_cuda:
        return hip_ops().order_stat_mean(deltas, t)
    srt = torch.sort(deltas, dim=0).values  # NaN sorts last
    acc = torch.zeros(deltas.shape[1], dtype=torch.float32)
    for k in range(t, K - t):  # ascending, fp32 adds
        acc += srt[k]
    return acc / torch.tensor(float(K - 2 * t), dtype=torch.float32)


def delta_gram(deltas: torch.Tensor) -> torch.Tensor:
    """G[a, b] = sum_i deltas[a, i] * deltas[b, i], fp32 [K, K]. GPU:
    f32-input MFMA over fixed coordinate ranges, partial tiles added in
    ascending order (bitwise symmetric, row-permutation equivariant,
    reproducible). CPU: float64 matmul rounded to fp32."""
    _check_stack(deltas)
    if deltas.is_cuda:
        return hip_ops().delta_gram(deltas)
    d = deltas.double()
    return (d @ d.t()).float()


def masked_wmean(deltas: torch.Tensor, weights: torch.Tensor
                 ) -> torch.Tensor:
    """sum_k w[k] * deltas[k] / sum(w) by fmaf in ascending k — the chain
    of weighted_fedavg with per-row addressing that is correct for every
    P. Rows with w[k] == 0 are skipped and never read."""
    _check_stack(deltas)
    if weights.shape != (deltas.shape[0],) or \
            weights.dtype != torch.float32:
        raise ValueError("weights must be a [K] fp32 tensor")
    if deltas.is_cuda:
        return hip_ops().masked_wmean(deltas, weights)
    acc = torch.zeros(deltas.shape[1], dtype=torch.float32)
    for k in range(deltas.shape[0]):  # fixed order, matches the kernel
        if float(weights[k]) == 0.0:
            continue
        acc += deltas[k] * weights[k]
    return acc * (torch.ones((), dtype=torch.float32) / weights.sum())
