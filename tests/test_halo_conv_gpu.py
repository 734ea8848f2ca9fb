"""Halo-tile pooled forward of conv2 (halo_conv_pool_kernel), bitwise.

The kernel keeps whole zero-ringed images in LDS and feeds the MFMA chain
of gemm256_kernel's single-slice pooled forward (taps ascending from +0,
then the all-zero tenth chunk) into that kernel's POOL epilogue, so both
outputs must be BITWISE what

    conv2d_fwd(x, w, b, 1, 1, relu=True) -> maxpool2d_fwd(2, 2, True)

gives wherever that forward runs unsplit: torch.equal, no tolerance.

The route only takes shapes whose fwd_pool plan has one K slice (a
split-K launch sums its slices in another order, so there the old kernel
and its pooling reduce stay). The planner splits K for every small batch
- at C = 32, Kout = 64 all of (5,6,6), (3,14,14), (9,14,14) and (2,22,22)
plan S = 3, and (1,2,2) with its 4 rows has no GEMM plan at all - so a
small geometric case cannot reach the kernel through the route and has
no unsplit oracle of its own size. Each gated
case therefore runs twice against ONE oracle per (H, W), computed once on
a batch just large enough to plan S == 1 (asserted through
conv_plan_route):

  * the case's own N images, the first N of that batch, through the
    kernel pinned with impl="halo_mfma" (geometry gate only), against
    the oracle's first N images - a row's chain does not depend on the
    batch around it;
  * the whole batch through the default route, which must report
    "halo_mfma", against the whole oracle.

BFLC_HALO_CONV is read once per process, so the gate-off side of the
model-level comparison runs in a fresh child process, once per module.
"""
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPO = Path(__file__).resolve().parent.parent
C, KOUT = 32, 64
W_SHAPE = [KOUT, 3, 3, C]
MODEL_BATCH = 96
NAMES = ["c1w", "c1b", "c2w", "c2b", "f1w", "f1b", "f2w", "f2b"]


def hip():
    from bflc_amd.ops import functional as fn
    return fn.hip_ops()


def bf(x):
    return x.to(DEV, torch.bfloat16).contiguous()


def group_images(h, w):
    """G: images the kernel stages per LDS group at this geometry."""
    return hip().halo_conv_group_images([1, h, w, C], W_SHAPE, 1, 1)


def unsplit_batch(h, w, at_least=1):
    """Smallest power-of-two batch >= at_least whose pooled forward plans
    one K slice on the double-buffered kernel."""
    n = 1
    while True:
        if n >= at_least:
            path, _, _, s, _ = hip().conv_plan_route(
                "fwd_pool", [n, h, w, C], W_SHAPE, 1, 1)
            if path == "gemm256" and s == 1:
                return n
        n *= 2
        assert n <= 1 << 16, (h, w)


def rand_inputs(n, h, w, c, kout, r, seed):
    """Asymmetric weights; half the channels get a bias low enough that
    many pool windows are all zero after ReLU (ties -> idx 0)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, c, generator=g)
    wt = torch.randn(kout, r, r, c, generator=g) / math.sqrt(r * r * c)
    b = torch.randn(kout, generator=g) * 0.5
    b[::2] -= 1.5
    return bf(x), bf(wt), bf(b)


def two_op(x, wt, b, stride, pad):
    y = hip().conv2d_fwd(x, wt, b, stride, pad, True)
    return hip().maxpool2d_fwd(y, 2, 2, True)


_ORACLE = {}


def oracle(h, w, at_least=1):
    """(x, w, b, y_pooled, idx) of the unsplit batch at (h, w): computed
    once per geometry and never written to afterwards."""
    key = (h, w)
    if key not in _ORACLE or _ORACLE[key][0].shape[0] < at_least:
        nb = unsplit_batch(h, w, at_least)
        x, wt, b = rand_inputs(nb, h, w, C, KOUT, 3, seed=1000 * h + w)
        yp, idx = two_op(x, wt, b, 1, 1)
        dead = (yp == 0)
        frac = dead.float().mean().item()
        assert 0.1 < frac < 0.95, frac
        assert (idx[dead] == 0).all()
        assert (yp > 0).any() and (idx > 0).any()
        _ORACLE[key] = (x, wt, b, yp, idx)
    return _ORACLE[key]


def assert_gated(n, h, w, max_blocks=0):
    x, wt, b, yp_ref, idx_ref = oracle(h, w, at_least=n)
    nb = x.shape[0]
    # the case's own N images through the pinned kernel
    xn = x[:n].contiguous()
    for _ in range(2):
        yp = hip().conv2d_relu_pool_fwd(xn, wt, b, 1, 1, max_blocks,
                                        "halo_mfma")
        assert torch.equal(yp, yp_ref[:n])
        yp, idx = hip().conv2d_relu_pool_fwd_idx(xn, wt, b, 1, 1, max_blocks,
                                                 "halo_mfma")
        assert torch.equal(yp, yp_ref[:n])
        assert torch.equal(idx, idx_ref[:n])
    # the unsplit batch through the default route
    xs = [nb, h, w, C]
    assert hip().conv2d_relu_pool_route(xs, W_SHAPE, 1, 1) == "gemm256_pool"
    assert hip().conv_fwd_pool_impl(xs, W_SHAPE, 1, 1) == "halo_mfma"
    yp = hip().conv2d_relu_pool_fwd(x, wt, b, 1, 1, max_blocks)
    assert torch.equal(yp, yp_ref)
    yp, idx = hip().conv2d_relu_pool_fwd_idx(x, wt, b, 1, 1, max_blocks)
    assert torch.equal(yp, yp_ref) and torch.equal(idx, idx_ref)
    # the old kernel, pinned, gives the same bits on the same batch
    yp, idx = hip().conv2d_relu_pool_fwd_idx(x, wt, b, 1, 1, 0, "gemm256")
    assert torch.equal(yp, yp_ref) and torch.equal(idx, idx_ref)


# (N, H, W): one window, every tap on the ring | 36 rows per image: MFMA
# tiles cross images, last tile partial | workload geometry
@pytest.mark.parametrize("case", [(1, 2, 2), (5, 6, 6), (3, 14, 14)],
                         ids=lambda c: "x".join(map(str, c)))
def test_halo_bitwise(case):
    assert_gated(*case)


def test_halo_n_below_group():
    """(3, 14, 14) is meant as N below G, but G follows the LDS and
    staging budgets: run G - 1 images (at least one) as well."""
    g = group_images(14, 14)
    assert g >= 1
    assert_gated(max(1, g - 1), 14, 14)


def test_halo_persistent_ragged():
    """4G + 1 images on two blocks: several groups per block, both LDS
    buffers, a ragged last group."""
    g = group_images(14, 14)
    assert g >= 1
    assert_gated(4 * g + 1, 14, 14, max_blocks=2)


# the largest (H, W) the gate admits: one image fills the staging slots
LARGEST = (22, 22)


def test_halo_largest_geometry():
    h, w = LARGEST
    assert group_images(h, w) == 1
    assert_gated(2, h, w)


@pytest.mark.parametrize("hw", [(22, 24), (24, 24)],
                         ids=lambda c: "x".join(map(str, c)))
def test_one_step_beyond_is_gemm256(hw):
    h, w = hw
    assert group_images(h, w) == 0
    nb = unsplit_batch(h, w)
    xs = [nb, h, w, C]
    assert hip().conv2d_relu_pool_route(xs, W_SHAPE, 1, 1) == "gemm256_pool"
    assert hip().conv_fwd_pool_impl(xs, W_SHAPE, 1, 1) == "gemm256"
    x, wt, b = rand_inputs(nb, h, w, C, KOUT, 3, seed=7)
    yp_ref, idx_ref = two_op(x, wt, b, 1, 1)
    yp, idx = hip().conv2d_relu_pool_fwd_idx(x, wt, b, 1, 1)
    assert torch.equal(yp, yp_ref) and torch.equal(idx, idx_ref)
    with pytest.raises(RuntimeError):
        hip().conv2d_relu_pool_fwd(x, wt, b, 1, 1, 0, "halo_mfma")


# (N, H, W, C, Kout, R, stride, pad) just outside the gate
OUTSIDE = {
    "C16": (64, 14, 14, 16, 64, 3, 1, 1),
    "C64": (64, 14, 14, 64, 64, 3, 1, 1),
    "Kout128": (64, 14, 14, 32, 128, 3, 1, 1),
    "stride2": (64, 16, 16, 32, 64, 3, 2, 1),
    "5x5": (64, 14, 14, 32, 64, 5, 1, 2),
    "splitK": (8, 8, 8, 32, 64, 3, 1, 1),
}


@pytest.mark.parametrize("name", list(OUTSIDE))
def test_outside_gate_is_gemm256(name):
    n, h, w, c, kout, r, stride, pad = OUTSIDE[name]
    xs, ws = [n, h, w, c], [kout, r, r, c]
    assert hip().conv_fwd_pool_impl(xs, ws, stride, pad) == "gemm256"
    if name == "splitK":
        path, _, _, s, _ = hip().conv_plan_route("fwd_pool", xs, ws, stride,
                                                 pad)
        assert path == "gemm256" and s > 1
    x, wt, b = rand_inputs(n, h, w, c, kout, r, seed=11)
    yp_ref, idx_ref = two_op(x, wt, b, stride, pad)
    yp = hip().conv2d_relu_pool_fwd(x, wt, b, stride, pad)
    assert torch.equal(yp, yp_ref)
    yp, idx = hip().conv2d_relu_pool_fwd_idx(x, wt, b, stride, pad)
    assert torch.equal(yp, yp_ref) and torch.equal(idx, idx_ref)


# ------------------------------------------------------------ model level

def model_outputs(batch):
    """Grad-free logits and one training step's gradients of FemnistCNN."""
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
    x = bf(torch.randn(batch, 28, 28, 1, generator=g))
    y = torch.randint(0, 62, (batch,), generator=g).to(DEV)
    with torch.no_grad():
        logits = m.forward(x).detach().clone()
    m.zero_grad()
    m.loss(x, y).backward()
    out = {f"grad.{k}": m.p(k).grad.detach().clone() for k in NAMES}
    out["logits"] = logits
    return out


def as_bits(t):
    t = t.contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return t.cpu().numpy()


def conv2_impl(batch):
    return hip().conv_fwd_pool_impl([batch, 14, 14, C], W_SHAPE, 1, 1)


def child_main(out):
    res = {"impl": np.array(conv2_impl(MODEL_BATCH))}
    for k, v in model_outputs(MODEL_BATCH).items():
        res[k] = as_bits(v)
    np.savez(out, **res)


@pytest.fixture(scope="module")
def gate_off(tmp_path_factory):
    out = tmp_path_factory.mktemp("halo_conv") / "gate_off.npz"
    env = dict(os.environ, BFLC_HALO_CONV="0", BFLC_FUSED_POOL="1",
               BFLC_FUSED_POOL_TRAIN="1",
               PYTHONPATH=os.pathsep.join(
                   [str(REPO)] + os.environ.get("PYTHONPATH", "").split(
                       os.pathsep)).rstrip(os.pathsep))
    subprocess.run([sys.executable, __file__, "--child", str(out)],
                   check=True, env=env, timeout=300)
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


def test_femnist_cnn_gate_on_vs_off(gate_off, monkeypatch):
    """Logits and all eight gradients of one step at batch 96, gate on
    (this process) against BFLC_HALO_CONV=0 (the child): bitwise."""
    monkeypatch.setenv("BFLC_FUSED_POOL", "1")
    monkeypatch.setenv("BFLC_FUSED_POOL_TRAIN", "1")
    assert str(gate_off["impl"]) == "gemm256"
    assert conv2_impl(MODEL_BATCH) == "halo_mfma"
    outs = model_outputs(MODEL_BATCH)
    for k, v in outs.items():
        assert v.float().abs().sum() > 0, k
        assert np.array_equal(as_bits(v), gate_off[k]), k


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    child_main(sys.argv[2])
