"""The grad-free conv stack as one kernel (halo_conv_stack_kernel), bitwise.

conv_relu_pool_stack_fwd(x, w1, b1, w2, b2) is conv3x3 + bias + ReLU +
2x2 pool twice (stride 1, pad 1). Where the first layer would take the
thin pooled route and the second the halo kernel, one kernel runs both:
each block computes its conv2 input images from the raw pixels into LDS
with the thin kernel's own per-output chain, then feeds the halo kernel's
MFMA chain. The result must be BITWISE

    conv2d_fwd(relu) -> maxpool2d_fwd -> conv2d_fwd(relu) -> maxpool2d_fwd

wherever conv1 runs the thin kernel's chain and conv2 runs unsplit:
torch.equal, no tolerance.

As in test_halo_conv_gpu.py, small geometric cases cannot reach the
kernel through the route (the thin route wants 65536 conv1 rows, the halo
gate an unsplit conv2 plan), so there is ONE oracle per (H1, W1), computed
once on a batch just large enough for both (asserted through
conv2d_relu_pool_route and conv_plan_route) and never written to
afterwards. A case's own N images, the first N of that batch, go through
the kernel pinned with impl="halo_stack" (geometry gate only) against the
oracle's first N - an image's chains do not depend on the batch around
it - and the whole batch goes through the default route, which must
report "halo_stack".

The oracle's conv1 is conv2d_fwd's unpooled thin kernel, which still runs
K padded to 16 taps; gemm_thin_conv_pool_kernel and the stack's stage run
nine taps and one `+ 0.f`. The signed-zero case pins that these are the
same bits where it could matter: all-(+0) and all-(-0) images under
all-negative / all-positive channels with -0.0 and +0.0 biases, compared
as int16 bit patterns.

BFLC_HALO_STACK is read once per process, so the gate-off side of the
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
K1, K2 = 32, 64
W1_SHAPE = [K1, 3, 3, 1]
W2_SHAPE = [K2, 3, 3, K1]
MODEL_BATCH = 96


def hip():
    from bflc_amd.ops import functional as fn
    return fn.hip_ops()


def bf(x):
    return x.to(DEV, torch.bfloat16).contiguous()


def bits(t):
    t = t.contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return t.cpu().numpy()


def group_images(h1, w1):
    """G: images a block of the stack kernel computes per LDS group."""
    return hip().halo_stack_group_images([1, h1, w1, 1], W1_SHAPE, W2_SHAPE)


def routes_ok(n, h1, w1):
    """conv1 thin and conv2 an unsplit gemm256 plan at this batch."""
    if hip().conv2d_relu_pool_route([n, h1, w1, 1], W1_SHAPE, 1,
                                    1) != "thin_pool":
        return False
    path, _, _, s, _ = hip().conv_plan_route(
        "fwd_pool", [n, h1 // 2, w1 // 2, K1], W2_SHAPE, 1, 1)
    return path == "gemm256" and s == 1


def gated_batch(h1, w1, at_least=1):
    n = 1
    while True:
        if n >= at_least and routes_ok(n, h1, w1):
            return n
        n *= 2
        assert n <= 1 << 17, (h1, w1)


def rand_params(seed, k1=K1, k2=K2):
    """Asymmetric weights of both signs; half the channels of each layer
    get a bias low enough that many pool windows are all zero after
    ReLU."""
    g = torch.Generator().manual_seed(seed)
    w1 = torch.randn(k1, 3, 3, 1, generator=g) / 3.0
    b1 = torch.randn(k1, generator=g) * 0.5
    b1[::2] -= 1.5
    w2 = torch.randn(k2, 3, 3, k1, generator=g) / math.sqrt(9 * k1)
    b2 = torch.randn(k2, generator=g) * 0.5
    b2[::2] -= 1.5
    return w1, b1, w2, b2


def two_op(x, w, b):
    y = hip().conv2d_fwd(x, w, b, 1, 1, True)
    return hip().maxpool2d_fwd(y, 2, 2, False)[0]


def two_op_twice(x, w1, b1, w2, b2):
    h = two_op(x, w1, b1)
    return h, two_op(h, w2, b2)


def dead_and_live(t):
    frac = (t == 0).float().mean().item()
    assert 0.05 < frac < 0.95, frac
    assert (t > 0).any()


_ORACLE = {}


def oracle(h1, w1, at_least=1):
    """(x, w1, b1, w2, b2, h_pooled, y) of the gated batch at (h1, w1)."""
    key = (h1, w1)
    if key not in _ORACLE or _ORACLE[key][0].shape[0] < at_least:
        nb = gated_batch(h1, w1, at_least)
        assert routes_ok(nb, h1, w1)
        g = torch.Generator().manual_seed(1000 * h1 + w1)
        x = bf(torch.randn(nb, h1, w1, 1, generator=g))
        p = [bf(t) for t in rand_params(seed=77 * h1 + w1)]
        h, y = two_op_twice(x, *p)
        dead_and_live(h)
        dead_and_live(y)
        _ORACLE[key] = (x, *p, h, y)
    return _ORACLE[key]


def assert_gated(n, h1, w1, max_blocks=0):
    x, w1t, b1, w2t, b2, _, y_ref = oracle(h1, w1, at_least=n)
    nb = x.shape[0]
    assert group_images(h1, w1) >= 1
    xn = x[:n].contiguous()
    for _ in range(2):
        y = hip().conv_relu_pool_stack_fwd(xn, w1t, b1, w2t, b2, max_blocks,
                                           "halo_stack")
        assert y.shape == (n, h1 // 4, w1 // 4, K2)
        assert torch.equal(y, y_ref[:n])
    # the whole batch through the default route
    assert hip().conv_relu_pool_stack_route(
        [nb, h1, w1, 1], W1_SHAPE, W2_SHAPE) == "halo_stack"
    for _ in range(2):
        y = hip().conv_relu_pool_stack_fwd(x, w1t, b1, w2t, b2, max_blocks)
        assert torch.equal(y, y_ref)
    # the two calls, pinned, give the same bits on the same batch
    y = hip().conv_relu_pool_stack_fwd(x, w1t, b1, w2t, b2, 0, "two_call")
    assert torch.equal(y, y_ref)


# (N, H1, W1): conv2 sees 2x2, every tap of both layers on a ring | MFMA
# tiles cross images, last tile partial | workload geometry
@pytest.mark.parametrize("case", [(1, 4, 4), (5, 12, 12), (3, 28, 28)],
                         ids=lambda c: "x".join(map(str, c)))
def test_stack_bitwise(case):
    assert_gated(*case)


def test_stack_n_below_group():
    g = group_images(28, 28)
    assert g >= 1
    assert_gated(max(1, g - 1), 28, 28)


def test_stack_persistent_ragged():
    """4G + 1 images on two blocks: several groups per block, both LDS
    buffers, a ragged last group."""
    g = group_images(28, 28)
    assert g >= 1
    assert_gated(4 * g + 1, 28, 28, max_blocks=2)


def test_stack_largest_geometry():
    """The largest raw image the geometry admits (conv2 at 22x22): one
    image a group, the LDS budget nearly full."""
    assert group_images(44, 44) == 1
    assert_gated(2, 44, 44)


def test_signed_zero_dropped_taps():
    """Nine taps and one `+ 0.f` against the sixteen-tap chain, where a
    signed zero could tell them apart."""
    h1 = w1 = 28
    nb = gated_batch(h1, w1, at_least=4)
    g = torch.Generator().manual_seed(31)
    x = torch.randn(nb, h1, w1, 1, generator=g)
    x[0] = 0.0
    x[1] = -0.0
    w1t, b1, w2t, b2 = rand_params(seed=32)
    assert (w1t > 0).any() and (w1t < 0).any()
    w1t[0] = -w1t[0].abs() - 0.01   # all negative, bias -0.0
    w1t[1] = -w1t[1].abs() - 0.01   # all negative, bias +0.0
    w1t[2] = w1t[2].abs() + 0.01    # all positive, bias -0.0
    w1t[3] = w1t[3].abs() + 0.01    # all positive, bias +0.0
    b1[0], b1[1], b1[2], b1[3] = -0.0, 0.0, -0.0, 0.0
    x, w1t, b1, w2t, b2 = bf(x), bf(w1t), bf(b1), bf(w2t), bf(b2)
    assert bits(b1)[0] == -32768 and bits(b1)[1] == 0
    assert bits(x[1]).min() == -32768 and bits(x[1]).max() == -32768
    h_ref, y_ref = two_op_twice(x, w1t, b1, w2t, b2)
    xs = [nb, h1, w1, 1]
    assert hip().conv2d_relu_pool_route(xs, W1_SHAPE, 1, 1) == "thin_pool"
    h = hip().conv2d_relu_pool_fwd(x, w1t, b1, 1, 1)
    assert np.array_equal(bits(h), bits(h_ref))
    h, idx = hip().conv2d_relu_pool_fwd_idx(x, w1t, b1, 1, 1)
    assert np.array_equal(bits(h), bits(h_ref))
    assert hip().conv_relu_pool_stack_route(xs, W1_SHAPE,
                                            W2_SHAPE) == "halo_stack"
    for impl in ("", "halo_stack"):
        y = hip().conv_relu_pool_stack_fwd(x, w1t, b1, w2t, b2, 0, impl)
        assert np.array_equal(bits(y), bits(y_ref)), impl


def test_non_finite_conv1_outputs():
    """The folded tail of the shared chain against the literal one. A NaN
    conv output fails the pool's `f > best` and is skipped, four of them
    leave -inf, and -inf itself is ReLU'd to 0: an all-NaN image, an
    all-(+inf) image (NaN under mixed-sign channels, +inf under an
    all-positive one, 0 under an all-negative one), one with a single
    +inf pixel and one with a single NaN pixel, conv1's pooled output
    compared as bit patterns with the two-op oracle. The stack is compared
    with its own two calls: same conv2 chain on the same conv2 input."""
    h1 = w1 = 28
    nb = gated_batch(h1, w1, at_least=8)
    g = torch.Generator().manual_seed(41)
    x = torch.randn(nb, h1, w1, 1, generator=g)
    x[0] = float("nan")
    x[1] = float("inf")
    x[2, 13, 13] = float("inf")
    x[3, 0, 27] = float("nan")
    x[4, 5, 5] = float("-inf")
    w1t, b1, w2t, b2 = rand_params(seed=42)
    w1t[0] = w1t[0].abs() + 0.01
    w1t[1] = -w1t[1].abs() - 0.01
    x, w1t, b1, w2t, b2 = bf(x), bf(w1t), bf(b1), bf(w2t), bf(b2)
    h_ref = two_op(x, w1t, b1)
    assert torch.isinf(h_ref.float()).any()
    assert (h_ref.float() == float("-inf")).any()
    assert not torch.isnan(h_ref.float()).any()
    xs = [nb, h1, w1, 1]
    assert hip().conv2d_relu_pool_route(xs, W1_SHAPE, 1, 1) == "thin_pool"
    h = hip().conv2d_relu_pool_fwd(x, w1t, b1, 1, 1)
    assert np.array_equal(bits(h), bits(h_ref))
    h, _ = hip().conv2d_relu_pool_fwd_idx(x, w1t, b1, 1, 1)
    assert np.array_equal(bits(h), bits(h_ref))
    y_ref = hip().conv_relu_pool_stack_fwd(x, w1t, b1, w2t, b2, 0, "two_call")
    y = hip().conv_relu_pool_stack_fwd(x, w1t, b1, w2t, b2, 0, "halo_stack")
    assert np.array_equal(bits(y), bits(y_ref))


# (N, H1, W1, Kout1, Kout2, pinned kernel refuses the geometry)
OUTSIDE = {
    "Kout1_16": (128, 28, 28, 16, 64, True),
    "Kout2_128": (128, 28, 28, 32, 128, True),
    "H1_30": (128, 30, 28, 32, 64, True),
    "below_thin_gate": (64, 28, 28, 32, 64, False),
    "past_halo_geom": (32, 44, 48, 32, 64, True),
}


@pytest.mark.parametrize("name", list(OUTSIDE))
def test_outside_gate_is_two_call(name):
    n, h1, w1, k1, k2, refuses = OUTSIDE[name]
    xs, w1s, w2s = [n, h1, w1, 1], [k1, 3, 3, 1], [k2, 3, 3, k1]
    assert hip().conv_relu_pool_stack_route(xs, w1s, w2s) == "two_call"
    if name == "below_thin_gate":
        assert hip().conv2d_relu_pool_route(xs, w1s, 1, 1) != "thin_pool"
    if name == "past_halo_geom":
        assert hip().halo_stack_group_images(xs, w1s, w2s) == 0
        assert group_images(44, 44) == 1
    g = torch.Generator().manual_seed(11)
    x = bf(torch.randn(n, h1, w1, 1, generator=g))
    w1t, b1, w2t, b2 = [bf(t) for t in rand_params(12, k1, k2)]
    _, y_ref = two_op_twice(x, w1t, b1, w2t, b2)
    y = hip().conv_relu_pool_stack_fwd(x, w1t, b1, w2t, b2)
    assert torch.equal(y, y_ref)
    if refuses:
        with pytest.raises(RuntimeError):
            hip().conv_relu_pool_stack_fwd(x, w1t, b1, w2t, b2, 0,
                                           "halo_stack")


# ------------------------------------------------------------ model level

def model_logits(batch):
    """Grad-free logits of FemnistCNN."""
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
    with torch.no_grad():
        return m.forward(x).detach().clone()


def stack_route(batch):
    return hip().conv_relu_pool_stack_route([batch, 28, 28, 1], W1_SHAPE,
                                            W2_SHAPE)


def child_main(out):
    np.savez(out, route=np.array(stack_route(MODEL_BATCH)),
             logits=bits(model_logits(MODEL_BATCH)))


@pytest.fixture(scope="module")
def gate_off(tmp_path_factory):
    out = tmp_path_factory.mktemp("halo_stack") / "gate_off.npz"
    env = dict(os.environ, BFLC_HALO_STACK="0", BFLC_HALO_CONV="1",
               BFLC_FUSED_POOL="1",
               PYTHONPATH=os.pathsep.join(
                   [str(REPO)] + os.environ.get("PYTHONPATH", "").split(
                       os.pathsep)).rstrip(os.pathsep))
    subprocess.run([sys.executable, __file__, "--child", str(out)],
                   check=True, env=env, timeout=300)
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


def test_femnist_cnn_gate_on_vs_off(gate_off, monkeypatch):
    """Grad-free logits at batch 96, stack on (this process) against
    BFLC_HALO_STACK=0 (the child): bitwise."""
    monkeypatch.setenv("BFLC_FUSED_POOL", "1")
    assert str(gate_off["route"]) == "two_call"
    assert stack_route(MODEL_BATCH) == "halo_stack"
    logits = model_logits(MODEL_BATCH)
    assert logits.shape == (MODEL_BATCH, 62)
    assert logits.float().abs().sum() > 0
    assert np.array_equal(bits(logits), gate_off["logits"])


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    child_main(sys.argv[2])
