"""Order-preserving fused weight gradient of the thin pooled first layer.

thin_conv_pool_wgrad_fused builds the operands of the materialised
chain's split-K GEMM (masked unpooled dy, im2col rows of x) in
registers and feeds them to the same mfma_f32_16x16x32_bf16 chain per
(K slice, 16-row fragment), then runs the same fixed-order reduce; db
comes from the unpool kernel's own walk without the plane store. So
(dw, db) must be BITWISE what

    pool_relu_bwd_colsum -> conv2d_bwd(x, w, dyf, stride, pad, None,
                                       False, False)

gives on the same inputs: torch.equal, no tolerance. Every case asserts
the split-K plan it was chosen for (through gemm_plan_route, so a planner
change cannot silently shrink the coverage) and that the default route
really ran the fused kernel. BFLC_THIN_FUSED_WGRAD is read once per
process, so the gate-off side (impl query and one model step) runs in a
fresh child process, once for the module.
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

# (N, H, W, Kout, pad): (S, kslice) of plan_dense(Kout, 16, Mpix) and the
# pixels of the last slice
CASES = {
    (1, 4, 4, 8, 1): (1, 32, 16),      # direct bf16 store, partial k-step
    (3, 6, 6, 8, 1): (4, 32, 12),      # steps straddle rows and images
    (5, 6, 6, 8, 1): (3, 64, 52),      # one full step + 20
    (2, 6, 10, 32, 1): (4, 32, 24),    # H != W
    (2, 28, 28, 32, 0): (22, 64, 8),   # pad 0
    (2, 28, 28, 64, 1): (25, 64, 32),  # four fragments, tail = one step
    (97, 28, 28, 32, 0): (410, 160, 132),
    (84, 28, 28, 32, 1): (412, 160, 96),
}
MODEL_BATCHES = (16, 96)
NAMES = ["c1w", "c1b", "c2w", "c2b", "f1w", "f1b", "f2w", "f2b"]


def hip():
    from bflc_amd.ops import functional as fn
    return fn.hip_ops()


def bf(x):
    return x.to(DEV, torch.bfloat16).contiguous()


def rand_inputs(n, h, w, c, kout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, c, generator=g)
    wt = torch.randn(kout, 3, 3, c, generator=g) / math.sqrt(9 * c)
    b = torch.randn(kout, generator=g) * 0.5
    return bf(x), bf(wt), bf(b)


def two_op_fwd(x, w, b, stride, pad):
    y = hip().conv2d_fwd(x, w, b, stride, pad, True)
    yp, idx = hip().maxpool2d_fwd(y, 2, 2, True)
    return y, yp, idx


def out_hw(h, w, pad):
    return h + 2 * pad - 2, w + 2 * pad - 2


def assert_plan(case):
    n, h, w, kout, pad = case
    oh, ow = out_hw(h, w, pad)
    mpix = n * oh * ow
    path, _, _, s, kslice = hip().gemm_plan_route(kout, 16, mpix, True, False)
    want_s, want_kslice, want_tail = CASES[case]
    assert path == "small" and (s, kslice) == (want_s, want_kslice)
    assert mpix - (s - 1) * kslice == want_tail


def assert_fused_bitwise(x, wt, yp, idx, dy, pad):
    """Both entries against the materialised chain, each run twice."""
    xs, ws = list(x.shape), list(wt.shape)
    assert hip().thin_pool_wgrad_impl(xs, ws, 1, pad, False) == "fused_mfma"
    assert hip().thin_pool_wgrad_impl(xs, ws, 1, pad, True) == "materialized"
    assert hip().conv2d_relu_pool_bwd_route(xs, ws, 1, pad, False,
                                            False) == "unpool"
    n, ph, pw, kout = yp.shape
    dyf, db_ref = hip().pool_relu_bwd_colsum(yp, idx, dy,
                                             [n, 2 * ph, 2 * pw, kout])
    _, dw_ref, _ = hip().conv2d_bwd(x, wt, dyf, 1, pad, None, False, False)
    assert dw_ref.shape == wt.shape
    for _ in range(2):
        dw, db = hip().thin_conv_pool_wgrad_fused(x, yp, idx, dy, 1, pad)
        assert torch.equal(dw.view(wt.shape), dw_ref)
        assert torch.equal(db, db_ref)
        dx, dw2, db2 = hip().conv2d_relu_pool_bwd(x, wt, yp, idx, dy, 1, pad,
                                                  True, False, False)
        assert dx.numel() == 0
        assert torch.equal(dw2, dw_ref) and torch.equal(db2, db_ref)
    return dw_ref, db_ref


@pytest.mark.parametrize("case", list(CASES), ids=lambda c: "x".join(map(str, c)))
def test_fused_wgrad_bitwise(case):
    n, h, w, kout, pad = case
    assert_plan(case)
    x, wt, b = rand_inputs(n, h, w, 1, kout, seed=29)
    _, yp, idx = two_op_fwd(x, wt, b, 1, pad)
    g = torch.Generator().manual_seed(31)
    dy = bf(torch.randn(yp.shape, generator=g))
    dw_ref, db_ref = assert_fused_bitwise(x, wt, yp, idx, dy, pad)
    assert dw_ref.float().abs().sum() > 0 and db_ref.float().abs().sum() > 0


@pytest.mark.parametrize("case", [(3, 6, 6, 8, 1), (84, 28, 28, 32, 1)],
                         ids=lambda c: "x".join(map(str, c)))
def test_fused_wgrad_negative_zero_and_dead_relu(case):
    """-0.0 in the pooled dy (the unpool stores +0 for it) and a bias low
    enough that most of y is ReLU-dead (those positions must be +0
    whatever dy holds)."""
    n, h, w, kout, pad = case
    assert_plan(case)
    x, wt, _ = rand_inputs(n, h, w, 1, kout, seed=43)
    b = bf(torch.full((kout,), -1.5))
    _, yp, idx = two_op_fwd(x, wt, b, 1, pad)
    dead = (yp == 0).float().mean().item()
    assert 0.5 < dead < 1.0, dead
    g = torch.Generator().manual_seed(47)
    dyc = torch.randn(yp.shape, generator=g)
    dyc[torch.rand(yp.shape, generator=g) < 0.2] = -0.0
    dy = bf(dyc)
    neg_zero = (dy.view(torch.int16) == -32768)
    assert neg_zero.any() and (neg_zero & (yp > 0)).any()
    dw_ref, _ = assert_fused_bitwise(x, wt, yp, idx, dy, pad)
    assert dw_ref.float().abs().sum() > 0


# ------------------------------------------------------------ model level

def model_grads(batch):
    """Gradients of one FemnistCNN loss.backward() at this batch size."""
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
    m.zero_grad()
    m.loss(x, y).backward()
    return {k: m.p(k).grad.detach().clone() for k in NAMES}


def as_bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy()


def child_main(out):
    """Gate-off side: impl queries of every case and the model grads."""
    res = {}
    for i, (n, h, w, kout, pad) in enumerate(CASES):
        impl = hip().thin_pool_wgrad_impl([n, h, w, 1], [kout, 3, 3, 1], 1,
                                          pad, False)
        res[f"impl.{i}"] = np.array(impl)
    for batch in MODEL_BATCHES:
        for k, v in model_grads(batch).items():
            res[f"grad.{batch}.{k}"] = as_bits(v)
    np.savez(out, **res)


@pytest.fixture(scope="module")
def gate_off(tmp_path_factory):
    out = tmp_path_factory.mktemp("thin_fused") / "gate_off.npz"
    env = dict(os.environ, BFLC_THIN_FUSED_WGRAD="0",
               BFLC_THIN_DIRECT_WGRAD="0", BFLC_FUSED_POOL_TRAIN="1",
               PYTHONPATH=os.pathsep.join(
                   [str(REPO)] + os.environ.get("PYTHONPATH", "").split(
                       os.pathsep)).rstrip(os.pathsep))
    subprocess.run([sys.executable, __file__, "--child", str(out)],
                   check=True, env=env, timeout=300)
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


def test_gate_off_is_materialized(gate_off):
    for i in range(len(CASES)):
        assert str(gate_off[f"impl.{i}"]) == "materialized"


@pytest.mark.parametrize("batch", MODEL_BATCHES)
def test_femnist_cnn_step_gate_on_vs_off(gate_off, monkeypatch, batch):
    """All eight gradients of one training step, gate on (this process)
    against gate off (the child): bitwise. Batch 96 is the smallest of
    the two at which conv1's forward takes the fused thin route, so that
    its backward reaches the fused kernel; batch 16 stays on the two-op
    path and must not move either."""
    monkeypatch.setenv("BFLC_FUSED_POOL_TRAIN", "1")
    monkeypatch.setenv("BFLC_THIN_DIRECT_WGRAD", "0")
    xs, ws = [batch, 28, 28, 1], [32, 3, 3, 1]
    assert hip().thin_pool_wgrad_impl(xs, ws, 1, 1, False) == "fused_mfma"
    if batch == 96:
        assert hip().conv2d_relu_pool_route(xs, ws, 1, 1) == "thin_pool"
    grads = model_grads(batch)
    for k in NAMES:
        assert grads[k].float().abs().sum() > 0, k
        assert np.array_equal(as_bits(grads[k]), gate_off[f"grad.{batch}.{k}"]), k


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    child_main(sys.argv[2])
