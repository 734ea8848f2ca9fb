"""Fused conv + bias + ReLU + 2x2 maxpool (grad-free forward) and the
guard-free conv GEMM staging loop: every result is compared BITWISE.

- The fused op against the two native kernels it replaces,
  maxpool2d_fwd(conv2d_fwd(..., relu=True), 2, 2, want_idx=False), with
  the route query asserted so nothing passes through the fallback
  unnoticed.
- conv2d_fwd and one dense GEMM against outputs recorded from the
  commit before the staging loop changed (tests/golden/
  conv_fwd_parent.npz, inputs regenerated exactly by det()).

The small gemm256 shapes are a handful of tiles, so the dispatcher
splits K for them (K = 288 runs as 3 slices at M = 512); the pooled
route follows the same tile / split-K choice and pools in its own
reduce, which is what keeps it bitwise. The scoring shapes run S = 1.
"""
import math
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = Path(__file__).parent / "golden" / "conv_fwd_parent.npz"


def hip():
    from bflc_amd.ops import functional as fn
    return fn.hip_ops()


def det(shape, seed, scale):
    """Machine-independent pseudo-random tensor: integer hash -> k*scale,
    |k| <= 127 and scale a power of two, so every value is exact in
    bf16 on any host."""
    n = math.prod(shape)
    i = torch.arange(n, dtype=torch.int64)
    h = (i * 2654435761 + seed * 40503 + 12345) % 2147483647
    k = (h >> 7) % 255 - 127
    return (k.to(torch.float32) * scale).reshape(shape)


def bf(x):
    return x.to(DEV, torch.bfloat16).contiguous()


# name: (N, H, W, C, Kout, stride, pad) — all 3x3
GEMM256_CASES = {
    # M = 512: full tiles only (interior staging); K = 288 ends in a
    # partial K-step
    "n8_8x8_c32_k64": (8, 8, 8, 32, 64, 1, 1),
    # M = 108: edge tiles with masked rows only
    "n3_6x6_c32_k64": (3, 6, 6, 32, 64, 1, 1),
    # M = 720: full tiles then a partial edge tile in one launch
    "n5_12x12_c32_k64": (5, 12, 12, 32, 64, 1, 1),
    # K = 72: one full K-step and one partial
    "n8_8x8_c8_k64": (8, 8, 8, 8, 64, 1, 1),
    # K = 576: nine exact K-steps, no partial
    "n8_8x8_c64_k64": (8, 8, 8, 64, 64, 1, 1),
    "n8_8x8_c32_k128": (8, 8, 8, 32, 128, 1, 1),
    # every pool window touches the zero padding
    "n8_4x4_c32_k64": (8, 4, 4, 32, 64, 1, 1),
    # M = 5904: enough tiles that K is not split, so the pooled
    # epilogue inside the GEMM kernel itself runs (the scoring-shape
    # path), full tiles + a short edge tile
    "n41_12x12_c32_k64": (41, 12, 12, 32, 64, 1, 1),
}
# cases recorded in the golden file (the last one was added for the
# pooled epilogue only)
GOLDEN_CASES = [k for k in GEMM256_CASES if k != "n41_12x12_c32_k64"]
DENSE_GEMM = (720, 288, 64)  # M edge + partial last K-step, CMODE 0


def conv_inputs(case, seed=0):
    n, h, w, c, kout, _, _ = case
    x = det((n, h, w, c), seed + 1, 1.0 / 64)
    wt = det((kout, 3, 3, c), seed + 2, 1.0 / 1024)
    b = det((kout,), seed + 3, 1.0 / 128)
    return bf(x), bf(wt), bf(b)


def unfused(x, w, b, stride, pad):
    y = hip().conv2d_fwd(x, w, b, stride, pad, True)
    return hip().maxpool2d_fwd(y, 2, 2, False)[0]


def route(x, w, stride, pad):
    return hip().conv2d_relu_pool_route(list(x.shape), list(w.shape),
                                        stride, pad)


def rand_inputs(n, h, w, c, kout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, c, generator=g)
    wt = torch.randn(kout, 3, 3, c, generator=g) / math.sqrt(9 * c)
    b = torch.randn(kout, generator=g) * 0.5
    return bf(x), bf(wt), bf(b)


@pytest.mark.parametrize("name", list(GEMM256_CASES))
def test_gemm256_pool_bitwise(name):
    n, h, w, c, kout, s, p = GEMM256_CASES[name]
    x, wt, b = rand_inputs(n, h, w, c, kout, seed=7)
    assert route(x, wt, s, p) == "gemm256_pool"
    y = hip().conv2d_relu_pool_fwd(x, wt, b, s, p)
    ref = unfused(x, wt, b, s, p)
    assert y.shape == ref.shape == (n, h // 2, w // 2, kout)
    assert torch.isfinite(ref.float()).all() and ref.float().abs().sum() > 0
    assert torch.equal(y, ref)


@pytest.mark.parametrize("n,pad", [(84, 1), (97, 0)])
def test_thin_pool_bitwise(n, pad):
    """Both just over the 65 536-row thin gate, which counts unpooled
    rows: pad 1 is M = 84 * 784 = 65 856; pad 0 gives OH = 26, where 84
    images are only 56 784 rows (below the gate the plain conv itself
    leaves the thin kernel for the MFMA one, so no thin route could be
    bitwise there) and 97 images are 65 572."""
    x, wt, b = rand_inputs(n, 28, 28, 1, 32, seed=11)
    assert route(x, wt, 1, pad) == "thin_pool"
    y = hip().conv2d_relu_pool_fwd(x, wt, b, 1, pad)
    ref = unfused(x, wt, b, 1, pad)
    oh = (28 + 2 * pad - 3 + 1) // 2
    assert y.shape == ref.shape == (n, oh, oh, 32)
    assert ref.float().abs().sum() > 0
    assert torch.equal(y, ref)


@pytest.mark.parametrize("n,h,c,kout,stride,pad", [
    (4, 7, 32, 64, 1, 1),    # odd OH/OW
    (16, 28, 1, 32, 1, 1),   # below the thin gate (M = 12 544)
    (4, 10, 32, 64, 2, 1),   # stride-2 conv, OH = 5
])
def test_fallback_bitwise(n, h, c, kout, stride, pad):
    x, wt, b = rand_inputs(n, h, h, c, kout, seed=13)
    assert route(x, wt, stride, pad) == "unfused"
    y = hip().conv2d_relu_pool_fwd(x, wt, b, stride, pad)
    assert torch.equal(y, unfused(x, wt, b, stride, pad))


def _golden():
    with np.load(GOLDEN) as z:
        return {k: torch.from_numpy(z[k].copy()) for k in z.files}


@pytest.fixture(scope="module")
def golden():
    return _golden()


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_conv_fwd_matches_recorded(name, golden):
    """Guard-free staging loop: conv2d_fwd is bitwise what it was."""
    case = GEMM256_CASES[name]
    x, wt, b = conv_inputs(case)
    y = hip().conv2d_fwd(x, wt, b, case[5], case[6], True)
    got = y.view(torch.int16).cpu().reshape(-1)
    assert torch.equal(got, golden[name].reshape(-1))


def test_dense_gemm_matches_recorded(golden):
    """The shared kernel's dense (CMODE 0) callers did not change."""
    m, k, n = DENSE_GEMM
    x = bf(det((m, k), 21, 1.0 / 64))
    w = bf(det((k, n), 22, 1.0 / 1024))
    b = bf(det((n,), 23, 1.0 / 128))
    y = hip().linear_fwd(x, w, b, True)
    got = y.view(torch.int16).cpu().reshape(-1)
    assert torch.equal(got, golden["dense_gemm"].reshape(-1))


def test_femnist_cnn_eval_logits_bitwise(monkeypatch):
    """FemnistCNN under no_grad at batch 96 (conv1 takes thin_pool,
    conv2 gemm256_pool): logits equal the A/B-gate-off path bitwise."""
    from bflc_amd.config import FLConfig
    from bflc_amd.models import build_model
    cfg = FLConfig.for_world(1, model="femnist_cnn", n_class=62,
                             samples_per_client=64, batch_size=32,
                             eval_samples=64)
    m = build_model(cfg, torch.device(DEV))
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():  # non-zero biases
        m.flat.add_(0.05 * torch.randn(m.numel, generator=g).to(DEV))
    m._sync_shadow()
    x = bf(torch.randn(96, 28, 28, 1, generator=g))
    assert route(x, m.p("c1w"), 1, 1) == "thin_pool"
    monkeypatch.setenv("BFLC_FUSED_POOL", "1")
    with torch.no_grad():
        fused = m.forward(x)
    monkeypatch.setenv("BFLC_FUSED_POOL", "0")
    with torch.no_grad():
        plain = m.forward(x)
    assert fused.shape == (96, 62)
    assert torch.isfinite(fused.float()).all()
    assert torch.equal(fused, plain)
    # training forwards are the two-op sequence whatever the gate says
    monkeypatch.setenv("BFLC_FUSED_POOL", "1")
    y = m.forward(x)
    assert y.requires_grad and torch.equal(y.detach(), plain)
